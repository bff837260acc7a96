"""Float64 reference of the per-step attention / decoder kernels (csrc/attention.hip) in plain torch, written from the
reference project's formulas (src/module.py:179-258 BaseAttention / ScaleDotAttention / LocationAwareAttention,
src/asr.py:277-313 Attention.forward, src/asr.py:218 the 1-step nn.LSTM, src/asr.py:103-109 nn.Embedding) - never from
the kernels - and the case tables shared by tests/test_attention_plan_cpu.py, tests/test_attention_reference_cpu.py and
tests/test_attention_variants_gpu.py.

Shapes: BN = B * N rows ordered (batch, head).  prev [B,N,T], Wc [K,N,2ks+1], c [B,T,K] (shared by the heads of a batch
row), key [BN,T,A], q [BN,A], Wp [A,K], we [A], be [1], value [BN,T,Dv], lens [B] (clamped to T).

Every function runs in the dtype of its arguments: the float64 run is the reference, the float32 run on the same inputs
gives e32 = helpers.rel_err(float32 run, float64 run), the rounding scale of the bound.

Criterion of the GPU test, per tensor: the hard limits of tests/test_cfg3_gpu.py - rel_err < 1e-3 on outputs, < 2e-3
on gradients - AND rel_err <= max(F * e32, 8 * 2**-24), F = 32 unless tests/test_attention_variants_gpu.py gives a
tensor kind its own factor with the cause beside it.

Energy rows name the launch geometry they exist for (fwd / bwd = (frames per workgroup, workgroups per row), None =
refused); tests/test_attention_plan_cpu.py holds every row to it through asrk_attn_energy_plan, so a re-tune of
energy_tpb or of the LDS budget moves SHAPES in this table, not assertions."""
import collections
import zlib

import torch
import torch.nn.functional as F

F64 = torch.float64
HARD_OUT, HARD_GRAD = 1e-3, 2e-3
FLOOR = 8 * 2.0 ** -24
FACTOR = 32


def bound(e32, kind, factor=FACTOR):
    """kind: the tensor's name; gradients are the names that start with 'd'"""
    return min(max(factor * e32, FLOOR), HARD_GRAD if kind.startswith('d') else HARD_OUT)


# ------------------------------------------------------------------------------------------------ the references
def loc_conv(prev, Wc):
    """Conv1d(N, K, 2ks+1, padding=ks) over the previous attention -> c [B,T,K]"""
    ks = (Wc.shape[-1] - 1) // 2
    return F.conv1d(prev, Wc, padding=ks).transpose(1, 2)


def loc_conv_grads(prev, Wc, dc):
    """-> dprev [B,N,T], dWc [K,N,2ks+1] by autograd"""
    p, w = prev.detach().clone().requires_grad_(True), Wc.detach().clone().requires_grad_(True)
    loc_conv(p, w).backward(dc)
    return p.grad, w.grad


def raw_energy(loc, key, q, c=None, Wp=None, we=None, be=None):
    """unscaled, unmasked energies [BN,T]: loc: we . tanh(key + q + tanh(Wp c)) + be; dot: key . q"""
    if not loc:
        return (key * q.unsqueeze(1)).sum(-1)
    N = key.shape[0] // c.shape[0]
    locf = torch.tanh(F.linear(c, Wp)).repeat_interleave(N, dim=0)                     # [BN,T,A]
    return F.linear(torch.tanh(key + q.unsqueeze(1) + locf), we.view(1, -1), be).squeeze(2)


def frame_mask(lens, N, T):
    """bool [BN,T]: frames t >= min(len, T)"""
    ln = lens.clamp(max=T).repeat_interleave(N)
    return torch.arange(T).unsqueeze(0) >= ln.unsqueeze(1)


def energy(loc, key, q, lens, temperature, c=None, Wp=None, we=None, be=None):
    """-> (e, attn): e = energies / temperature with -inf beyond the length, attn = softmax(e) (0 beyond)"""
    BN, T, _ = key.shape
    N = BN // lens.shape[0]
    e = (raw_energy(loc, key, q, c, Wp, we, be) / temperature).masked_fill(frame_mask(lens, N, T), float('-inf'))
    return e, torch.softmax(e, dim=-1)


def softmax_bwd(attn, dattn, lens, temperature):
    """de [BN,T] = attn * (dattn - sum_t attn * dattn) / temperature on the frames below the length, 0 beyond: the
    gradient of the raw energies for ANY attn row (for a true softmax row it is the softmax Jacobian)."""
    BN, T = attn.shape
    N = BN // lens.shape[0]
    dot = (attn * dattn).sum(-1, keepdim=True)
    de = attn * (dattn - dot) / temperature
    return de.masked_fill(frame_mask(lens, N, T), 0.0)


def energy_bwd(loc, key, q, lens, temperature, attn, dattn, c=None, Wp=None, we=None, be=None):
    """-> dict dkey, dq (+ dc, dWp, dwe, dbe): de by hand (softmax_bwd), then autograd of the raw energies"""
    de = softmax_bwd(attn, dattn, lens, temperature)
    names = ('key', 'q') + (('c', 'Wp', 'we', 'be') if loc else ())
    vals = dict(key=key, q=q, c=c, Wp=Wp, we=we, be=be)
    leaf = {k: vals[k].detach().clone().requires_grad_(True) for k in names}
    raw_energy(loc, **leaf).backward(de)
    out = {'d' + k: v.grad for k, v in leaf.items()}
    out['de'] = de
    return out


def context(attn, value):
    """attn [BN,T], value [BN,T,Dv] -> ctx [BN,Dv]"""
    return torch.bmm(attn.unsqueeze(1), value).squeeze(1)


def context_bwd(dctx, value):
    """-> dattn [BN,T]"""
    return torch.bmm(value, dctx.unsqueeze(2)).squeeze(2)


def lstm_cell(gates, c_prev):
    """pre-activations [B,4H] (i, f, g, o) -> (activated gates, c, h)"""
    i, f, g, o = gates.chunk(4, dim=1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev + i * g
    return torch.cat([i, f, g, o], dim=1), c, o * torch.tanh(c)


def lstm_cell_bwd(gates, c_prev, dh, dc):
    """-> (dgates: gradient of the pre-activations, dc_prev) by autograd; dh / dc may be None"""
    g, cp = gates.detach().clone().requires_grad_(True), c_prev.detach().clone().requires_grad_(True)
    _, c, h = lstm_cell(g, cp)
    loss = 0
    if dh is not None:
        loss = loss + (h * dh).sum()
    if dc is not None:
        loss = loss + (c * dc).sum()
    loss.backward()
    return g.grad, cp.grad


def embedding(idx, W):
    """rows of W; an id outside [0, V) gives a zero row"""
    ok = (idx >= 0) & (idx < W.shape[0])
    return torch.where(ok.unsqueeze(1), W[idx.clamp(0, W.shape[0] - 1)], torch.zeros((), dtype=W.dtype))


def embedding_bwd(idx, dout, V):
    """-> dW [V,D]; ids outside [0, V) are ignored"""
    ok = (idx >= 0) & (idx < V)
    return torch.zeros(V, dout.shape[1], dtype=dout.dtype).index_add_(0, idx[ok], dout[ok])


def embedding_bwd_sequential_f32(idx, dout, base):
    """float32 accumulation in token order onto `base`: what the ordered kernel promises bit for bit"""
    out = base.clone()
    V = out.shape[0]
    for r, v in enumerate(idx.tolist()):
        if 0 <= v < V:
            out[v] += dout[r]
    return out


# ------------------------------------------------------------------------------------------------ case tables
ConvCase = collections.namedtuple('ConvCase', 'name B N T K ks skip why')
CONV_CASES = [
    ConvCase('c_t1', 1, 1, 1, 1, 0, '', 'T = 1, one tap, K = 1: waves 1-3 have no channel'),
    ConvCase('c_t63_k3', 3, 2, 63, 3, 3, '', 'T = 63: one ragged tile; K < 4'),
    ConvCase('c_t64_k4', 1, 4, 64, 4, 3, '', 'T = 64: exactly one tile; one channel per wave; one head per wave'),
    ConvCase('c_t65_k5_n5', 3, 5, 65, 5, 3, '', 'T = 65: second tile holds one frame; K = 5 and N = 5: wave 0 twice'),
    ConvCase('c_t130_ks100', 3, 1, 130, 10, 100, '', 'three tiles, 201 taps (the cfg3 filter), K = 10'),
    ConvCase('c_ks130_k16', 1, 2, 130, 16, 130, '', '261 taps > 256: the j += 256 loop of the weight gradient; K = 16'),
    ConvCase('c_ks_gt_t', 3, 2, 5, 3, 9, '', 'ks > T: every window is mostly padding'),
    ConvCase('c_k16_n4', 3, 4, 65, 16, 3, '', 'K = 16 with 4 heads'),
    ConvCase('c_no_dprev', 3, 2, 65, 5, 3, 'dprev', 'dprev_att == NULL'),
    ConvCase('c_no_dwc', 3, 2, 65, 5, 3, 'dWc', 'dWc_acc == NULL'),
]

EnergyCase = collections.namedtuple('EnergyCase', 'name loc B N T A K temp lens fwd bwd softmax why')


def _e(name, loc, B, N, T, A, K, temp, lens, fwd, bwd='same', softmax=False, why=''):
    return EnergyCase(name, loc, B, N, T, A, K if loc else 0, temp, tuple(lens), fwd, fwd if bwd == 'same' else bwd,
                      softmax, why)


def _energy_rows(loc):
    p = 'l_' if loc else 'd_'
    cyc = lambda pat, n: [pat[i % len(pat)] for i in range(n)]
    rows = [
        # lens: T, 1, a chunk boundary t0, t0 + 1, beyond T (clamped)
        _e(p + 'a1', loc, 5, 1, 9, 1, 1, 1.0, (9, 1, 5, 6, 12), (5, 2), why='A = 1; tpb 5: below 8, no multiple of 4'),
        _e(p + 'bn1_t9', loc, 1, 1, 9, 65, 10, 0.5, (6,), (5, 2), why='BN = 1: tpb 5; the length ends at t0 + 1'),
        _e(p + 'a63', loc, 5, 2, 70, 63, 10, 2.0, (70, 1, 64, 65, 75), (8, 9), why='A = 63; last chunk holds 6 frames'),
        _e(p + 'a64', loc, 5, 4, 70, 64, 16, 0.5, (70, 1, 64, 65, 75), (8, 9), why='A = 64; K = 16 (the dck limit); N = 4'),
        _e(p + 'a65', loc, 5, 1, 70, 65, 1, 1.0, (70, 1, 8, 9, 71), (8, 9), why='A = 65: one lane takes a second column'),
        _e(p + 'a257', loc, 5, 2, 33, 257, 10, 2.0, (33, 1, 14, 15, 40), (7, 5), why='A = 257 crosses the 256-thread tile; tpb 7'),
        _e(p + 'a300_t200', loc, 5, 1, 200, 300, 10, 0.5, (200, 1, 120, 121, 230), (8, 25), why='small BN, T = 200: 25 chunks'),
        _e(p + 'a300_n4', loc, 5, 4, 33, 300, 16, 1.0, (33, 1, 28, 29, 34), (7, 5), why='the cfg3 width with 4 heads, K = 16'),
        _e(p + 'bn1024', loc, 256, 4, 7, 8, 10, 2.0, cyc((7, 1, 3, 4, 9), 256), (7, 1), why='BN >= 1024: one chunk, tpb = T'),
        _e(p + 'tpb20', loc, 128, 4, 40, 63, 1, 1.0, cyc((40, 1, 20, 21, 44), 128), (20, 2), why='tpb 20, two chunks'),
        _e(p + 'softmax', loc, 5, 2, 70, 65, 10, 0.5, (70, 1, 64, 65, 75), (8, 9), softmax=True,
           why='a true softmax row: dbe vanishes'),
    ]
    if loc:
        rows += [
            _e('l_shrink', 1, 32, 4, 160, 424, 16, 1.0, cyc((160, 1, 80, 81, 170, 90, 10, 11), 32), (20, 8), (10, 16),
               why='backward LDS 10A + 5AK + tpb K > 38400 floats at tpb 20: shrunk to 10'),
            _e('l_k17_fwd', 1, 5, 1, 9, 20, 17, 1.0, (9, 1, 5, 6, 12), (5, 2), None, why='K = 17: forward runs, backward refuses'),
        ]
    else:
        rows += [
            _e('d_a600', 0, 5, 1, 33, 600, 0, 1.0, (33, 1, 14, 15, 40), (7, 5), why='dot attention wider than 512'),
            _e('d_a424_no_shrink', 0, 32, 4, 160, 424, 0, 1.0, cyc((160, 1, 80, 81, 170, 90, 10, 11), 32), (20, 8),
               why='the shrink row in dot mode: LDS 5A, tpb stays 20'),
        ]
    return rows


ENERGY_CASES = _energy_rows(1) + _energy_rows(0)
ENERGY_BY_NAME = {c.name: c for c in ENERGY_CASES}
# (loc, bwd, BN, T, A, K) -> status: what the plan and the launchers refuse on the host
ENERGY_REFUSED = [
    ((1, 1, 5, 9, 20, 17), -2, 'K = 17 on the loc backward: dck[16]'),
    ((1, 1, 4, 8, 430, 16), -2, 'backward LDS 38828 floats > 38400 even at tpb 8'),
    ((1, 0, 4, 8, 2400, 16), -2, 'forward LDS over 150 KB'),
    ((1, 0, 4, 8, 20, 0), -1, 'loc with K = 0'),
    ((0, 0, 4, 0, 20, 0), -1, 'T = 0'),
    ((0, 1, 4, 8, 0, 0), -1, 'A = 0'),
    ((0, 0, -1, 8, 20, 0), -1, 'BN < 0'),
]

CtxCase = collections.namedtuple('CtxCase', 'name BN T Dv pad why')
CTX_CASES = [
    CtxCase('x_d1_t1', 1, 1, 1, 0, 'the smallest call'),
    CtxCase('x_d255_pad', 6, 3, 255, 24, 'Dv = 255, row stride Dv + 24'),
    CtxCase('x_d256', 6, 5, 256, 0, 'Dv = 256: exactly one thread tile'),
    CtxCase('x_d257_t257_pad', 6, 257, 257, 24, 'second thread tile holds one column; T = 257 > 256 staging threads'),
    CtxCase('x_d600_bn1', 1, 257, 600, 0, 'three thread tiles, BN = 1'),
    CtxCase('x_d600_pad', 6, 5, 600, 24, 'three thread tiles with a padded row stride'),
]

CELL_SHAPES = [(3, 5), (1, 256), (7, 37), (128, 64)]
CELL_MODES = ('both', 'dh', 'dc')
EMB_SHAPES = [(1, 1, 1), (7, 300, 31), (130, 10, 5), (513, 33, 1031)]

ChainCase = collections.namedtuple('ChainCase', 'name loc N')
CHAIN_CASES = [ChainCase('loc_n1', 1, 1), ChainCase('loc_n2', 1, 2), ChainCase('loc_n4', 1, 4), ChainCase('dot_n1', 0, 1),
               ChainCase('dot_n4', 0, 4)]
CHAIN = dict(B=3, T=70, lens=(70, 33, 1), A=20, Dv=40, K=3, ks=4, temp=0.7, L=3)


# ------------------------------------------------------------------------------------------------ inputs
_inputs = {}


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _cached(name, make):
    if name not in _inputs:
        _inputs[name] = make(_gen(name))
    return _inputs[name]


def conv_inputs(c):
    """float32 CPU tensors, seeded by the row's name, made once and never modified.  R* are the pre-fills of += buffers."""
    def make(g):
        KW = 2 * c.ks + 1
        return dict(prev=torch.softmax(2 * torch.randn(c.B, c.N, c.T, generator=g), dim=-1),
                    Wc=torch.randn(c.K, c.N, KW, generator=g) / (c.N * KW) ** 0.5,
                    dc=torch.randn(c.B, c.T, c.K, generator=g),
                    RdWc=torch.randn(c.K, c.N, KW, generator=g))
    return _cached(c.name, make)


def conv_reference_of(c, t, dtype=F64):
    prev, Wc, dc = (t[k].to(dtype) for k in ('prev', 'Wc', 'dc'))
    dprev, dWc = loc_conv_grads(prev, Wc, dc)
    return dict(c=loc_conv(prev, Wc), dprev=dprev, dWc=dWc)


def half_mass_rows(lens, N, T, g):
    """[BN,T] float32: positive below the length, exactly 0 beyond, every row sums to 0.5 (not a softmax: dbe != 0)"""
    BN = len(lens) * N
    a = torch.rand(BN, T, generator=g, dtype=F64) + 0.05
    a = a.masked_fill(frame_mask(torch.tensor(lens), N, T), 0.0)
    return (0.5 * a / a.sum(-1, keepdim=True)).float()


def energy_inputs(c):
    def make(g):
        BN = c.B * c.N
        t = dict(key=torch.tanh(torch.randn(BN, c.T, c.A, generator=g)),
                 q=torch.randn(BN, c.A, generator=g) * (1.0 if c.loc else c.A ** -0.5),
                 lens=torch.tensor(c.lens, dtype=torch.int64),
                 dattn=torch.randn(BN, c.T, generator=g),
                 Rdkey=torch.randn(BN, c.T, c.A, generator=g))
        if c.loc:
            t.update(c=torch.randn(c.B, c.T, c.K, generator=g) * 0.5,
                     Wp=torch.randn(c.A, c.K, generator=g) / c.K ** 0.5,
                     we=torch.randn(c.A, generator=g) / c.A ** 0.5,
                     be=torch.randn(1, generator=g) * 0.1,
                     RdWp=torch.randn(c.A, c.K, generator=g), Rdwe=torch.randn(c.A, generator=g),
                     Rdbe=torch.randn(1, generator=g))
        if c.softmax:
            t['attn'] = energy_forward_of(c, t)['attn'].float()
        else:
            t['attn'] = half_mass_rows(c.lens, c.N, c.T, g)
        return t
    return _cached(c.name, make)


def _loc_args(c, t, dtype):
    return {k: t[k].to(dtype) for k in ('c', 'Wp', 'we', 'be')} if c.loc else {}


def energy_forward_of(c, t, dtype=F64):
    e, attn = energy(c.loc, t['key'].to(dtype), t['q'].to(dtype), t['lens'], c.temp, **_loc_args(c, t, dtype))
    return dict(e=e, attn=attn)


def energy_backward_of(c, t, dtype=F64):
    return energy_bwd(c.loc, t['key'].to(dtype), t['q'].to(dtype), t['lens'], c.temp, t['attn'].to(dtype),
                      t['dattn'].to(dtype), **_loc_args(c, t, dtype))


def ctx_inputs(c):
    def make(g):
        lens = [(c.T, 1, c.T // 2 + 1, c.T, 2, c.T)[i % 6] for i in range(c.BN)]
        lens = [min(max(v, 1), c.T) for v in lens]
        a = torch.softmax(torch.randn(c.BN, c.T, generator=g), dim=-1)
        a = a.masked_fill(frame_mask(torch.tensor(lens), 1, c.T), 0.0)
        return dict(attn=a, value=torch.randn(c.BN, c.T, c.Dv, generator=g), dctx=torch.randn(c.BN, c.Dv, generator=g))
    return _cached(c.name, make)


def ctx_reference_of(c, t, dtype=F64):
    return dict(ctx=context(t['attn'].to(dtype), t['value'].to(dtype)), dattn=context_bwd(t['dctx'].to(dtype), t['value'].to(dtype)))


def cell_inputs(B, H):
    def make(g):
        gates = torch.randn(B, 4 * H, generator=g) * 2
        flat = gates.view(-1)
        for i, v in enumerate((30.0, -30.0, 90.0, -90.0) * 4):        # saturated pre-activations in every gate kind
            flat[(i * 7919) % flat.numel()] = v
        return dict(gates=gates, c_prev=torch.randn(B, H, generator=g), dh=torch.randn(B, H, generator=g),
                    dc=torch.randn(B, H, generator=g))
    return _cached('cell_%d_%d' % (B, H), make)


def cell_reference_of(t, mode, dtype=F64):
    gates, c_prev = t['gates'].to(dtype), t['c_prev'].to(dtype)
    act, c, h = lstm_cell(gates, c_prev)
    dg, dcp = lstm_cell_bwd(gates, c_prev, t['dh'].to(dtype) if mode in ('both', 'dh') else None,
                            t['dc'].to(dtype) if mode in ('both', 'dc') else None)
    return dict(gates=act, cell=c, h=h, dgates=dg, dc_prev=dcp)


def emb_inputs(n, D, V):
    def make(g):
        idx = torch.randint(0, V, (n,), generator=g)
        if n >= 7:
            idx[1], idx[3] = -1, V                      # out of range on both sides
            idx[4] = idx[5] = idx[0]                    # repeated ids
        return dict(idx=idx, W=torch.randn(V, D, generator=g), dout=torch.randn(n, D, generator=g),
                    RdW=torch.randn(V, D, generator=g))
    return _cached('emb_%d_%d_%d' % (n, D, V), make)


def emb_reference_of(t, dtype=F64):
    return dict(emb=embedding(t['idx'], t['W'].to(dtype)), dW=embedding_bwd(t['idx'], t['dout'].to(dtype), t['W'].shape[0]))


# ------------------------------------------------------------------------------------------------ the chained steps
CHAIN_PARAMS = ('q0', 'q1', 'q2', 'prev0', 'key', 'value', 'Wc', 'Wp', 'we', 'be')


def chain_inputs(cc):
    def make(g):
        s = CHAIN
        B, T, A, Dv, K, ks, N = s['B'], s['T'], s['A'], s['Dv'], s['K'], s['ks'], cc.N
        BN = B * N
        lens = torch.tensor(s['lens'], dtype=torch.int64)
        prev0 = torch.softmax(torch.randn(B, N, T, generator=g), dim=-1)
        prev0 = prev0.masked_fill(frame_mask(lens, N, T).view(B, N, T), 0.0)
        t = dict(key=torch.tanh(torch.randn(BN, T, A, generator=g)), value=torch.randn(BN, T, Dv, generator=g),
                 lens=lens, prev0=prev0, g_ctx0=torch.randn(BN, Dv, generator=g), g_ctx2=torch.randn(BN, Dv, generator=g),
                 g_attn2=torch.randn(B, N, T, generator=g),
                 Wc=torch.randn(K, N, 2 * ks + 1, generator=g) / (N * (2 * ks + 1)) ** 0.5,
                 Wp=torch.randn(A, K, generator=g) / K ** 0.5, we=torch.randn(A, generator=g) / A ** 0.5 * 3,
                 be=torch.randn(1, generator=g) * 0.1)
        for l in range(s['L']):
            t['q%d' % l] = torch.randn(BN, A, generator=g) * (1.0 if cc.loc else A ** -0.5 * 3)
        return t
    return _cached('chain_' + cc.name, make)


def chain_forward(cc, p, lens):
    """p: dict of tensors (any dtype, possibly requiring grad) -> lists attn_l [B,N,T], ctx_l [BN,Dv]; attn_l is the
    prev_att of step l + 1"""
    s = CHAIN
    B, N, T = s['B'], cc.N, s['T']
    prev, attns, ctxs = p['prev0'], [], []
    for l in range(s['L']):
        kw = dict(c=loc_conv(prev, p['Wc']), Wp=p['Wp'], we=p['we'], be=p['be']) if cc.loc else {}
        _, attn = energy(cc.loc, p['key'], p['q%d' % l], lens, s['temp'], **kw)
        ctxs.append(context(attn, p['value']))
        prev = attn.view(B, N, T)
        attns.append(prev)
    return attns, ctxs


def chain_loss(t, attns, ctxs, dtype):
    """the contexts of steps 0 and 2 and the attention of step 2: step 1 is used through the chain only"""
    return ((ctxs[0] * t['g_ctx0'].to(dtype)).sum() + (ctxs[2] * t['g_ctx2'].to(dtype)).sum()
            + (attns[2] * t['g_attn2'].to(dtype)).sum())


def chain_params(cc):
    return [k for k in CHAIN_PARAMS if cc.loc or k not in ('prev0', 'Wc', 'Wp', 'we', 'be')]


def chain_reference_of(cc, t, dtype=F64):
    """-> dict attn0..2, ctx0..2 and d<param> for chain_params(cc), by autograd"""
    p = {k: t[k].to(dtype).clone().requires_grad_(True) for k in chain_params(cc)}
    if not cc.loc:
        p['prev0'] = t['prev0'].to(dtype)
    attns, ctxs = chain_forward(cc, p, t['lens'])
    chain_loss(t, attns, ctxs, dtype).backward()
    out = {'attn%d' % l: a.detach() for l, a in enumerate(attns)}
    out.update({'ctx%d' % l: c.detach() for l, c in enumerate(ctxs)})
    # dot energies do not read prev_att: step 1 then reaches nothing in the loss and its q has no gradient
    out.update({'d' + k: torch.zeros_like(p[k]) if p[k].grad is None else p[k].grad for k in chain_params(cc)})
    return out


def chain_manual_grads(cc, t, dtype=F64):
    """-> (the same gradients from the per-step references chained by hand (context_bwd, energy_bwd, loc_conv_grads),
    the sum over steps of sum |de|: the scale of the rounding noise that is all a true softmax leaves of dbe)"""
    s = CHAIN
    B, N, T, L = s['B'], cc.N, s['T'], s['L']
    p = {k: t[k].to(dtype) for k in CHAIN_PARAMS}
    with torch.no_grad():
        attns, _ = chain_forward(cc, p, t['lens'])
    prevs = [p['prev0']] + attns[:-1]
    g_ctx = [t['g_ctx0'].to(dtype), None, t['g_ctx2'].to(dtype)]
    g = {'d' + k: torch.zeros_like(p[k]) for k in chain_params(cc)}
    dattn_next = t['g_attn2'].to(dtype).reshape(B * N, T)
    de_abs = 0.0
    for l in reversed(range(L)):
        attn = attns[l].reshape(B * N, T)
        dattn = dattn_next.clone()
        if g_ctx[l] is not None:
            dattn = dattn + context_bwd(g_ctx[l], p['value'])
            g['dvalue'] += attn.unsqueeze(2) * g_ctx[l].unsqueeze(1)
        kw = dict(c=loc_conv(prevs[l], p['Wc']), Wp=p['Wp'], we=p['we'], be=p['be']) if cc.loc else {}
        r = energy_bwd(cc.loc, p['key'], p['q%d' % l], t['lens'], s['temp'], attn, dattn, **kw)
        g['dkey'] += r['dkey']
        g['dq%d' % l] = r['dq']
        de_abs += float(r['de'].abs().sum())
        if cc.loc:
            for k in ('dWp', 'dwe', 'dbe'):
                g[k] += r[k]
            dprev, dWc = loc_conv_grads(prevs[l], p['Wc'], r['dc'])
            g['dWc'] += dWc
            dattn_next = dprev.reshape(B * N, T)
            if l == 0:
                g['dprev0'] = dprev
        else:
            dattn_next = torch.zeros_like(dattn)
    return g, de_abs


def cell_chain_inputs():
    def make(g):
        B, In, H = 5, 13, 9
        return dict(w_ih=torch.randn(4 * H, In, generator=g) / In ** 0.5, w_hh=torch.randn(4 * H, H, generator=g) / H ** 0.5,
                    b_ih=torch.randn(4 * H, generator=g) * 0.1, b_hh=torch.randn(4 * H, generator=g) * 0.1,
                    x0=torch.randn(B, In, generator=g), x1=torch.randn(B, In, generator=g), x2=torch.randn(B, In, generator=g),
                    h0=torch.randn(B, H, generator=g) * 0.5, c0=torch.randn(B, H, generator=g) * 0.5,
                    g_h0=torch.randn(B, H, generator=g), g_h2=torch.randn(B, H, generator=g), g_c2=torch.randn(B, H, generator=g))
    return _cached('cell_chain', make)


CELL_CHAIN_PARAMS = ('x0', 'x1', 'x2', 'h0', 'c0', 'w_ih', 'w_hh', 'b_ih', 'b_hh')


def cell_chain_reference_of(t, dtype=F64):
    """three chained nn.LSTM steps on length-1 sequences; the middle step's output reaches the loss through the chain
    only -> dict h_last, cell_last and d<param>"""
    p = {k: t[k].to(dtype).clone().requires_grad_(True) for k in CELL_CHAIN_PARAMS}
    h, c, hs = p['h0'], p['c0'], []
    for l in range(3):
        gates = F.linear(p['x%d' % l], p['w_ih'], p['b_ih']) + F.linear(h, p['w_hh'], p['b_hh'])
        _, c, h = lstm_cell(gates, c)
        hs.append(h)
    ((hs[0] * t['g_h0'].to(dtype)).sum() + (hs[2] * t['g_h2'].to(dtype)).sum() + (c * t['g_c2'].to(dtype)).sum()).backward()
    out = dict(h_last=hs[2].detach(), cell_last=c.detach())
    out.update({'d' + k: v.grad for k, v in p.items()})
    return out
