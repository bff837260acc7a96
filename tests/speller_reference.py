"""Float64 reference of the teacher-forced attention-decoder loop (shared by tests/test_speller_reference_cpu.py,
tests/test_speller_plan_cpu.py and tests/test_speller_variants_gpu.py), written in plain torch with autograd from the
definitions oracle/asr_oracle.py: DecodeMemory.step restates - never from the code under test:

  * the first alignment of location-aware attention is uniform over the valid frames (1 / len_b);
  * the location features are a ZERO-padded convolution of the previous alignment, K kernels of 2 ks + 1 taps over
    all heads, projected to the attention width and squashed;
  * energies beyond lens[b] are -inf before the softmax, so those alignments are exactly 0;
  * the decoder is a stack of LSTM cells (rows i, f, g, o) or one GRU cell in nn.GRU's own layout (rows r, z, n);
  * several heads attend over rows b * N + n of key / value, their contexts are concatenated per utterance and go
    through merge_head.

loop_reference(...) takes the argument list of speller_ops.SpellerLoopFn.apply - except that a GRU decoder's weights
stay in nn.GRU's layout, the four-rows-per-unit stacking is the device side's business - and returns
(states [B,L,H], att_seq [B,N,L,Te]).  CASES / DOT_CASES / STEP_CASES are the shapes the GPU tests run, one or more
per kernel variant `make_plan` can select and per boundary between two variants; tests/test_speller_plan_cpu.py holds
every case to the variant named here."""
import collections
import math

import torch

F64 = torch.float64


def attention_step_reference(q, prev_att, key, value, lens, temperature, nhead=1, Wc=None, Wp=None, we=None, be=None):
    """one attention step.  q [B*N,A], prev_att [B,N,Te] (location-aware; None = the uniform first alignment), key
    [B*N,Te,A], value [B*N,Te,Dv], lens [B]; Wc [K,N,2ks+1] is None for dot-product energies.
    -> (attn [B,N,Te], per-head contexts [B*N,Dv])"""
    BN, Te, A = key.shape
    N = int(nhead)
    B = BN // N
    lens = lens.to(torch.int64).cpu()
    valid = torch.arange(Te).unsqueeze(0) < lens.unsqueeze(1)                     # [B,Te]
    if Wc is not None:
        if prev_att is None:
            prev_att = (valid.to(F64) / lens.to(F64).unsqueeze(1)).unsqueeze(1).repeat(1, N, 1)
        K, _, KW = Wc.shape
        ks = (KW - 1) // 2
        padded = torch.cat([prev_att.new_zeros(B, N, ks), prev_att, prev_att.new_zeros(B, N, ks)], dim=2)
        windows = padded.unfold(2, KW, 1)                                         # [B,N,Te,KW]: taps t - ks .. t + ks
        conv = torch.einsum('bntj,knj->btk', windows, Wc)                         # [B,Te,K]
        loc = torch.tanh(conv @ Wp.t())                                           # [B,Te,A]
        loc = loc.unsqueeze(1).expand(B, N, Te, A).reshape(BN, Te, A)             # every head adds the same features
        energy = torch.tanh(key + q.unsqueeze(1) + loc) @ we.reshape(A) + be.reshape(())
    else:
        energy = (key * q.unsqueeze(1)).sum(-1)
    row_valid = valid.unsqueeze(1).expand(B, N, Te).reshape(BN, Te)
    attn = torch.softmax((energy / temperature).masked_fill(~row_valid, -math.inf), dim=-1)
    ctx = (attn.unsqueeze(2) * value).sum(1)                                      # [B*N,Dv]
    return attn.view(B, N, Te), ctx


def lstm_cell_reference(x, h, c, w_ih, w_hh, b_ih, b_hh):
    i, f, g, o = (x @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh).chunk(4, dim=1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def gru_cell_reference(x, h, w_ih, w_hh, b_ih, b_hh):
    xr, xz, xn = (x @ w_ih.t() + b_ih).chunk(3, dim=1)
    hr, hz, hn = (h @ w_hh.t() + b_hh).chunk(3, dim=1)
    r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
    n = torch.tanh(xn + r * hn)
    return (1 - z) * n + z * h


def loop_reference(key, value, lens, sos_emb, teacher_emb, Wq, bq, Wc, Wp, we, be, W_ih, W_hh, b_ih, b_hh, L,
                   temperature, cell=0, nhead=1, Wm=None, bm=None, *upper):
    """the loop with tf_rate == 1: step 0 reads <sos>, step t > 0 teacher token t - 1; the query reads the states of
    all decoder layers side by side; `states` are the top layer's outputs"""
    d = lambda t: None if t is None else t.to(F64)
    key, value, sos_emb, teacher_emb, Wq, bq, Wc, Wp, we, be, W_ih, W_hh, b_ih, b_hh, Wm, bm = (
        d(t) for t in (key, value, sos_emb, teacher_emb, Wq, bq, Wc, Wp, we, be, W_ih, W_hh, b_ih, b_hh, Wm, bm))
    layers = [(W_ih, W_hh, b_ih, b_hh)] + [tuple(d(t) for t in upper[4 * i:4 * i + 4]) for i in range(len(upper) // 4)]
    N = int(nhead)
    BN, Te, A = key.shape
    B, Dv, H = BN // N, value.shape[2], W_hh.shape[1]
    h = [key.new_zeros(B, H) for _ in layers]
    c = [key.new_zeros(B, H) for _ in layers]
    prev, states, atts = None, [], []
    for t in range(L):
        q = torch.tanh(torch.cat(h, dim=1) @ Wq.t() + bq).view(BN, A)
        attn, ctx = attention_step_reference(q, prev, key, value, lens, temperature, N, Wc, Wp, we, be)
        prev = attn
        if N > 1:
            ctx = ctx.view(B, N * Dv) @ Wm.t() + bm
        x = torch.cat([sos_emb if t == 0 else teacher_emb[:, t - 1], ctx], dim=1)
        for l, w in enumerate(layers):
            if cell == 1:
                h[l] = gru_cell_reference(x, h[l], *w)
            else:
                h[l], c[l] = lstm_cell_reference(x, h[l], c[l], *w)
            x = h[l]
        states.append(x)
        atts.append(attn)
    return torch.stack(states, dim=1), torch.stack(atts, dim=2)


# ------------------------------------------------------------------------------------------------ the case table
H, E, L_STEPS, TEMPERATURE = 20, 8, 3, 0.7       # decoder width, embedding width, decode steps of every loop case
STAGED = (0, 0)                                  # attend_energy_kernel / energy_bwd_kernel2

# fwd / bwd: the <NA, KM> instantiation of attend_energy_kernel2 / energy_bwd_kernel3 the shape must get (STAGED: the
# staged kernel), None for dot-product attention; ctx_vec: the vector (True) or scalar (False) softmax/context kernel
Case = collections.namedtuple('Case', 'name B N Te A K taps Dv lens cell layers L fwd bwd ctx_vec')


def _lens(B, Te):
    """ragged: one utterance as long as the memory, one of a single frame, the rest in between"""
    if B == 1:
        return [Te]
    mid = [Te - 1 - (Te // 3 + i * 7919) % (Te - 2) for i in range(B - 2)]      # 2 <= len <= Te - 1, spread out
    return [Te] + mid + [1]


def _loc(name, B, Te, A, K, taps, Dv, fwd, bwd, cell=0, L=L_STEPS, lens=None):
    return Case(name, B, 1, Te, A, K, taps, Dv, lens or _lens(B, Te), cell, 1, L, fwd, bwd, Dv % 4 == 0)


def _dot(name, B, N, Te, A, Dv, layers=1):
    return Case(name, B, N, Te, A, 0, 0, Dv, _lens(B, Te), 0, layers, L_STEPS, None, None, Dv % 4 == 0)


CASES = [
    _loc('k1', 3, 21, 37, 1, 5, 12, (2, 12), (2, 12)),                  # K = 1: the a, k split has no reciprocal
    _loc('a128_k12', 3, 21, 128, 12, 9, 12, (2, 12), (2, 12)),          # both upper limits of <2,12>
    _loc('k13', 3, 21, 40, 13, 9, 12, (2, 16), (2, 16)),
    _loc('a129_k16', 3, 21, 129, 16, 9, 12, (5, 16), (5, 16)),
    _loc('a256_k16', 2, 19, 256, 16, 9, 10, (5, 16), (5, 16)),          # A K = 4096 exactly; scalar context kernel
    _loc('a320_k12', 2, 19, 320, 12, 9, 12, (5, 12), (5, 12)),          # A at its limit
    _loc('a320_k13', 2, 19, 320, 13, 9, 12, STAGED, STAGED),            # A K = 4160 > 4096
    _loc('a321', 2, 19, 321, 3, 9, 12, STAGED, STAGED),
    _loc('k17', 2, 19, 20, 17, 9, 12, STAGED, STAGED),
    _loc('taps255', 2, 21, 24, 4, 255, 12, (2, 12), (2, 12)),           # all four tap registers, window >> Te
    _loc('taps257', 2, 21, 24, 4, 257, 12, STAGED, (2, 12)),
    _loc('tpb32_km16', 32, 256, 16, 16, 9, 12, (2, 16), (2, 16)),       # tpb = 32: tpb KM = 512, every thread stages s_c
    _loc('tpb40', 32, 264, 16, 3, 9, 12, STAGED, STAGED),               # tpb > 32; Te > 224: context kernel past CTX_CF
    _loc('te1030', 1, 1030, 8, 3, 9, 12, (2, 12), STAGED, L=2),         # Te > 1024
    _loc('te1030_len1', 1, 1030, 8, 3, 9, 12, (2, 12), STAGED, L=2, lens=[1]),
    _loc('dv258', 2, 19, 24, 3, 9, 258, (2, 12), (2, 12)),              # scalar context kernel, two column blocks
    _loc('k13_gru', 3, 21, 40, 13, 9, 12, (2, 16), (2, 16), cell=1),
    _loc('a321_gru', 2, 19, 321, 3, 9, 12, STAGED, STAGED, cell=1),
]
TPB = {'tpb32_km16': (32, 32), 'tpb40': (40, 40)}      # frames per workgroup (forward, backward) the notes rely on

DOT_CASES = [
    _dot('dot_h1', 3, 1, 21, 65, 12),
    _dot('dot_h3_a512', 2, 3, 33, 512, 10),                             # A at DOT_NA's limit, scalar context kernel
    _dot('dot_h2_l2', 2, 2, 70, 37, 12, layers=2),                      # 2-layer LSTM decoder
]

# the per-step kernels (csrc/attention.hip): (name, mode, heads, B, Te, A, K, taps, Dv, lens)
StepCase = collections.namedtuple('StepCase', 'name mode N B Te A K taps Dv lens')
STEP_CASES = [StepCase('%s_h%d' % (n, N), 'loc', N, B, Te, A, K, taps, Dv, lens)
              for N in (1, 2)
              for n, B, Te, A, K, taps, Dv, lens in (('k1', 3, 21, 37, 1, 5, 10, _lens(3, 21)),
                                                      ('k16', 2, 70, 65, 16, 9, 12, _lens(2, 70)),
                                                      ('tiny', 1, 5, 4, 3, 21, 3, [5] if N == 1 else [1]))]
STEP_CASES += [StepCase('dot_h%d' % N, 'dot', N, 3, 33, 65, 0, 0, 12, _lens(3, 33)) for N in (1, 3)]
STEP_K17 = StepCase('k17', 'loc', 1, 2, 21, 20, 17, 9, 12, _lens(2, 21))      # backward refuses K > 16


def make_loop_inputs(case, seed=0):
    """-> dict of float32 CPU tensors in SpellerLoopFn.apply's argument order (a GRU's weights in nn.GRU's layout):
    key through tanh, weights scaled by 1 / sqrt(fan_in), plus the two output gradients g1 / g2"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = case
    BN, G = c.B * c.N, (3 if c.cell == 1 else 4)
    t = collections.OrderedDict()
    t['key'] = torch.tanh(rn(BN, c.Te, c.A))
    t['value'] = rn(BN, c.Te, c.Dv)
    t['sos_emb'] = rn(c.B, E)
    t['teacher_emb'] = rn(c.B, c.L, E)
    t['Wq'] = rn(c.N * c.A, c.layers * H) / math.sqrt(c.layers * H)
    t['bq'] = rn(c.N * c.A) * 0.1
    if c.K:
        t['Wc'] = rn(c.K, 1, c.taps) / math.sqrt(c.taps)
        t['Wp'] = rn(c.A, c.K) / math.sqrt(c.K)
        t['we'] = rn(1, c.A) / math.sqrt(c.A)
        t['be'] = rn(1) * 0.1
    t['W_ih'] = rn(G * H, E + c.Dv) / math.sqrt(E + c.Dv)
    t['W_hh'] = rn(G * H, H) / math.sqrt(H)
    t['b_ih'] = rn(G * H) * 0.1
    t['b_hh'] = rn(G * H) * 0.1
    if c.N > 1:
        t['Wm'] = rn(c.Dv, c.N * c.Dv) / math.sqrt(c.N * c.Dv)
        t['bm'] = rn(c.Dv) * 0.1
    for l in range(1, c.layers):
        t['W_ih_l%d' % l] = rn(4 * H, H) / math.sqrt(H)
        t['W_hh_l%d' % l] = rn(4 * H, H) / math.sqrt(H)
        t['b_ih_l%d' % l] = rn(4 * H) * 0.1
        t['b_hh_l%d' % l] = rn(4 * H) * 0.1
    return t, rn(c.B, c.L, H), rn(c.B, c.N, c.L, c.Te)


def loop_args(case, t, gru_layout=None):
    """the positional arguments of SpellerLoopFn.apply / loop_reference from make_loop_inputs' tensors; gru_layout:
    what turns nn.GRU's four parameters into the ones the callee takes (the device side's stack_gru_params)"""
    cellw = (t['W_ih'], t['W_hh'], t['b_ih'], t['b_hh'])
    if case.cell == 1 and gru_layout is not None:
        cellw = gru_layout(*cellw)
    upper = [t['%s_l%d' % (n, l)] for l in range(1, case.layers) for n in ('W_ih', 'W_hh', 'b_ih', 'b_hh')]
    return (t['key'], t['value'], torch.tensor(case.lens), t['sos_emb'], t['teacher_emb'], t['Wq'], t['bq'],
            t.get('Wc'), t.get('Wp'), t.get('we'), t.get('be'), *cellw, case.L, TEMPERATURE, case.cell, case.N,
            t.get('Wm'), t.get('bm'), *upper)
