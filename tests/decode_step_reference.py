"""Reference of ONE decode step (speller_ops.SpellerStepper / MultiSpellerStepper: query, location-aware energies,
masked softmax, context, decoder cell) in plain torch, float64 by default, built on attention_step_reference /
lstm_cell_reference / gru_cell_reference of tests/speller_reference.py - never on the code under test - and the case
table shared by tests/test_decode_step_plan_cpu.py, tests/test_decode_step_reference_cpu.py and
tests/test_decode_step_variants_gpu.py.

Rows attend over memory row_mem[i] of key [U,Te,A] / value [U,Te,Dv] / lens [U]; the context is computed per MEMORY
(the rows of a memory times its value matrix), value[row_mem] is never materialised.  A GRU's weights stay in nn.GRU's
layout (the device side stacks them, speller_ops.stack_gru_params).

Criterion of the GPU tests (bound): the project's hard limit helpers.rel_err < 1e-3, and the sharper
max(F * e32, 4 * 2**-24) capped at 1e-3, where e32 is rel_err of THIS function evaluated in float32 on the CPU against
its float64 run and F is set per tensor kind from one measurement on the device (tests/test_decode_step_variants_gpu.py
records the ratios)."""
import collections
import math

import torch

import speller_reference as R

F64 = torch.float64
TEMPERATURE = R.TEMPERATURE
STAGED = R.STAGED
HARD = 1e-3
FLOOR = 4 * 2.0 ** -24
LSTM_CELL_GEMM_ROWS = 128          # restated from decoder_ops (test_decode_step_plan_cpu holds the two together)


def bound(e32, F):
    return min(max(F * e32, FLOOR), HARD)


def context_per_memory(attn, value, row_mem):
    """attn [n,Te], value [U,Te,Dv], row_mem [n] -> ctx [n,Dv]: one small matrix product per memory"""
    ctx = attn.new_zeros(attn.shape[0], value.shape[2])
    for u in torch.unique(row_mem).tolist():
        rows = (row_mem == u).nonzero().flatten()
        ctx[rows] = attn[rows] @ value[u]
    return ctx


def step_reference(key, value, lens, row_mem, emb, prev_att, h, c, Wq, bq, Wc, Wp, we, be, W_ih, W_hh, b_ih, b_hh,
                   temperature=TEMPERATURE, cell=0, dtype=F64):
    """key [U,Te,A], value [U,Te,Dv], lens [U], row_mem [n] (None: row i -> memory i), emb [n,E], prev_att [n,1,Te],
    h / c [n,H] -> (attn [n,1,Te], ctx [n,Dv], h' [n,H], c' [n,H] or None for a GRU cell), computed in `dtype`"""
    d = lambda t: None if t is None else t.to(dtype)
    key, value, emb, prev_att, h, c, Wq, bq, Wc, Wp, we, be, W_ih, W_hh, b_ih, b_hh = (
        d(t) for t in (key, value, emb, prev_att, h, c, Wq, bq, Wc, Wp, we, be, W_ih, W_hh, b_ih, b_hh))
    n = h.shape[0]
    row_mem = torch.arange(n) if row_mem is None else row_mem.to(torch.int64).cpu()
    q = torch.tanh(h @ Wq.t() + bq)
    # energies and alignment of every row over ITS memory (the key rows are small; the value rows are not gathered)
    attn, _ = R.attention_step_reference(q, prev_att, key[row_mem], key.new_zeros(n, key.shape[1], 1),
                                         lens.cpu()[row_mem], temperature, 1, Wc, Wp, we, be)
    ctx = context_per_memory(attn[:, 0], value, row_mem)
    x = torch.cat([emb, ctx], dim=1)
    if cell == 1:
        return attn, ctx, R.gru_cell_reference(x, h, W_ih, W_hh, b_ih, b_hh), None
    h_new, c_new = R.lstm_cell_reference(x, h, c, W_ih, W_hh, b_ih, b_hh)
    return attn, ctx, h_new, c_new


# ------------------------------------------------------------------------------------------------ the case table
# stepper: 'multi' (MultiSpellerStepper) / 'shared' (SpellerStepper, all rows over ONE memory) / 'rows' (SpellerStepper,
# row i over memory i).  rg: asrk_speller_t::row_group; row_mem: None = arange(n) // rg (rg > 1) or arange(n).
# energy: the <NA, KM> instantiation of attend_energy_kernel2 the shape must get, STAGED = attend_energy_kernel.
# ctx: the softmax/context kernel ('scalar' / 'vector' / 'group'); branch: the cell branch of MultiSpellerStepper.step
# ('fused': inside asrk_speller_step_f32; 'gemm': three bf16x6 panel GEMMs + asrk_lstm_cell_fwd_f32).
# gpu False: the shape only pins a dispatch boundary on the CPU.  steps: chained steps the GPU test runs.
Case = collections.namedtuple('Case', 'name stepper n U rg row_mem Te A K taps Dv E H cell energy ctx branch gpu steps')

PERM = (2, 0, 1, 1, 2, 0, 2)


def _m(name, n, U, rg, Te, A, K, taps, Dv, E, H, cell, energy, ctx, branch, row_mem=None, gpu=True):
    return Case(name, 'multi', n, U, rg, row_mem, Te, A, K, taps, Dv, E, H, cell, energy, ctx, branch, gpu, 1)


def _s(name, stepper, n, Te, A, K, taps, Dv, cell, energy, ctx, steps=1):
    return Case(name, stepper, n, 1 if stepper == 'shared' else n, 0, None, Te, A, K, taps, Dv, 8, 20, cell, energy,
                ctx, 'fused', True, steps)


MULTI_CASES = [
    # non-monotonic indirection in attend_energy_kernel2 and the vector context kernel
    _m('m_perm', 7, 3, 0, 21, 37, 1, 5, 12, 8, 20, 0, (2, 12), 'vector', 'fused', row_mem=PERM),
    # ... in the staged energy kernel and the scalar context kernel
    _m('m_perm_staged', 7, 3, 0, 19, 321, 3, 9, 10, 8, 20, 1, STAGED, 'scalar', 'fused', row_mem=PERM),
    _m('m_rg2_gemm', 128, 64, 2, 21, 16, 3, 9, 32, 32, 32, 0, (2, 12), 'group', 'gemm'),    # smallest group + gemm
    _m('m_rg2_n126', 126, 63, 2, 21, 16, 3, 9, 32, 32, 32, 0, (2, 12), 'vector', 'fused'),  # one group short: 63 < 64
    _m('m_rg4_ragged', 130, 33, 4, 21, 16, 3, 9, 32, 32, 32, 0, (2, 12), 'vector', 'gemm'),  # B % RG != 0
    _m('m_rg2_dv30', 128, 64, 2, 21, 16, 3, 9, 30, 32, 32, 0, (2, 12), 'scalar', 'fused'),  # Dv % 4 != 0, Dv % 32 != 0
    # waves with 2 and 1 rows, Te > 64, Te % 8 = 6: the tail loop
    _m('m_rg9_te70', 72, 8, 9, 70, 16, 3, 9, 2048, 8, 20, 0, (2, 12), 'group', 'fused'),
    # idle waves, Te < 8: the tail loop only, Te % 4 != 0
    _m('m_rg5_te7', 80, 16, 5, 7, 8, 1, 5, 1024, 8, 20, 1, (2, 12), 'group', 'fused'),
    # production beam width, ragged last column block (the min(d0, Dv - 4) clamp), 512 rows through the fused cell
    _m('m_rg16_dv260', 512, 32, 16, 13, 24, 4, 5, 260, 8, 20, 0, (2, 12), 'group', 'fused'),
    # CG_MAXR rows per wave, group LDS exactly 64 KiB
    _m('m_rg32_te512', 256, 8, 32, 512, 8, 3, 9, 2048, 32, 32, 0, STAGED, 'group', 'gemm'),
    _m('m_rg32_te516', 256, 8, 32, 516, 8, 3, 9, 2048, 32, 32, 0, STAGED, 'vector', 'gemm', gpu=False),  # LDS over
    _m('m_rg33', 66, 2, 33, 21, 16, 3, 9, 2048, 8, 20, 0, (2, 12), 'vector', 'fused', gpu=False),  # RG > 8 * CG_MAXR
]

SINGLE_CASES = [
    _s('s_sh1_ae2', 'shared', 1, 21, 37, 1, 5, 12, 0, (2, 12), 'vector'),
    _s('s_sh16_ae2_gru', 'shared', 16, 21, 37, 1, 5, 12, 1, (2, 12), 'vector'),
    _s('s_sh1_staged_gru', 'shared', 1, 19, 321, 3, 9, 10, 1, STAGED, 'scalar'),
    _s('s_sh16_staged', 'shared', 16, 19, 321, 3, 9, 10, 0, STAGED, 'scalar'),
    _s('s_rows3', 'rows', 3, 21, 37, 1, 5, 12, 0, (2, 12), 'vector'),                       # ragged lengths, row i -> i
    _s('s_chain', 'shared', 16, 21, 37, 1, 5, 10, 0, (2, 12), 'scalar', steps=2),           # slot 1 -> slot 0
]

CASES = MULTI_CASES + SINGLE_CASES
GPU_MULTI = [c for c in MULTI_CASES if c.gpu]
GROUP_CASES = [c for c in GPU_MULTI if c.ctx == 'group']


def cell_branch(c):
    """the predicate of MultiSpellerStepper.step, restated"""
    many = (c.stepper == 'multi' and c.cell == 0 and c.n >= LSTM_CELL_GEMM_ROWS
            and c.E % 32 == 0 and c.Dv % 32 == 0 and c.H % 32 == 0)
    return 'gemm' if many else 'fused'


def row_mem_of(c):
    """-> int64 [n], or None where the stepper takes no indirection (SpellerStepper)"""
    if c.stepper != 'multi':
        return None
    if c.row_mem is not None:
        return torch.tensor(c.row_mem, dtype=torch.int64)
    return torch.arange(c.n) // max(c.rg, 1)


def memory_of_rows(c):
    """the memory every row attends over, whatever the stepper: int64 [n]"""
    if c.stepper == 'shared':
        return torch.zeros(c.n, dtype=torch.int64)
    rm = row_mem_of(c)
    return torch.arange(c.n) if rm is None else rm


def make_inputs(c, seed=5):
    """-> dict of float32 CPU tensors: memories (key through tanh), ragged lens per memory (speller_reference._lens),
    per-row emb / h / c, prev_att = a softmax over the valid frames of the row's memory, weights scaled by
    1 / sqrt(fan_in) with a GRU's in nn.GRU's layout"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    G = 3 if c.cell == 1 else 4
    t = collections.OrderedDict()
    t['key'] = torch.tanh(rn(c.U, c.Te, c.A))
    t['value'] = rn(c.U, c.Te, c.Dv)
    t['lens'] = torch.tensor(R._lens(c.U, c.Te), dtype=torch.int64)
    mem = memory_of_rows(c)
    valid = torch.arange(c.Te).unsqueeze(0) < t['lens'][mem].unsqueeze(1)
    t['emb'] = rn(c.n, c.E)
    t['prev_att'] = torch.softmax((rn(c.n, c.Te) * 2).masked_fill(~valid, -math.inf), dim=-1).unsqueeze(1)
    t['h'] = torch.tanh(rn(c.n, c.H))
    t['c'] = rn(c.n, c.H)
    t['Wq'] = rn(c.A, c.H) / math.sqrt(c.H)
    t['bq'] = rn(c.A) * 0.1
    t['Wc'] = rn(c.K, 1, c.taps) / math.sqrt(c.taps)
    t['Wp'] = rn(c.A, c.K) / math.sqrt(c.K)
    t['we'] = rn(1, c.A) / math.sqrt(c.A)
    t['be'] = rn(1) * 0.1
    t['W_ih'] = rn(G * c.H, c.E + c.Dv) / math.sqrt(c.E + c.Dv)
    t['W_hh'] = rn(G * c.H, c.H) / math.sqrt(c.H)
    t['b_ih'] = rn(G * c.H) * 0.1
    t['b_hh'] = rn(G * c.H) * 0.1
    return t


WEIGHTS = ('Wq', 'bq', 'Wc', 'Wp', 'we', 'be', 'W_ih', 'W_hh', 'b_ih', 'b_hh')


def reference_of(case, t, dtype=F64, **over):
    """step_reference on make_inputs' tensors (over: replacements, e.g. the second step's prev_att / h / c)
    -> dict attn / ctx / h / c (c absent for a GRU)"""
    a = dict(t, **over)
    attn, ctx, h, cc = step_reference(a['key'], a['value'], a['lens'], memory_of_rows(case), a['emb'], a['prev_att'],
                                      a['h'], a['c'], *[a[w] for w in WEIGHTS], TEMPERATURE, case.cell, dtype)
    out = dict(attn=attn, ctx=ctx, h=h)
    if cc is not None:
        out['c'] = cc
    return out
