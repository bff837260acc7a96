"""CPU: the decode-step reference (tests/decode_step_reference.py) is what it claims to be, and the GPU tests' limit can
see the defects the row-grouped softmax/context kernel invites: for every group case of the table the reference is
evaluated with ONE deliberate mutation of the context sum, and the context has to move by more than 1e-2 - ten times
the hard limit helpers.rel_err < 1e-3.  If a case falls below that, its inputs change, not the threshold."""
import math

import pytest
import torch

from helpers import rel_err
import decode_step_reference as D
import speller_reference as R

SHIFT = 1e-2
_cache = {}


def _base(c):
    """inputs and float64 reference of a case, computed once and shared (never modified)"""
    if c.name not in _cache:
        t = D.make_inputs(c)
        _cache[c.name] = (t, D.reference_of(c, t))
    return _cache[c.name]


def test_step_reference_equals_a_per_row_loop_over_gathered_memories():
    """against the plainest form of the same step: every row alone, its memory gathered, no batching"""
    c = next(c for c in D.CASES if c.name == 'm_perm')
    t, ref = _base(c)
    mem = D.memory_of_rows(c)
    w = {k: t[k].double() for k in D.WEIGHTS}
    for i in range(c.n):
        u = int(mem[i])
        q = torch.tanh(t['h'][i:i + 1].double() @ w['Wq'].t() + w['bq'])
        attn, ctx = R.attention_step_reference(q, t['prev_att'][i:i + 1].double(), t['key'][u:u + 1].double(),
                                               t['value'][u:u + 1].double(), t['lens'][u:u + 1], D.TEMPERATURE, 1,
                                               w['Wc'], w['Wp'], w['we'], w['be'])
        h, cc = R.lstm_cell_reference(torch.cat([t['emb'][i:i + 1].double(), ctx], 1), t['h'][i:i + 1].double(),
                                      t['c'][i:i + 1].double(), w['W_ih'], w['W_hh'], w['b_ih'], w['b_hh'])
        for name, got in (('attn', attn), ('ctx', ctx), ('h', h), ('c', cc)):
            assert rel_err(ref[name][i:i + 1], got) < 1e-12, (name, i)


def test_inputs_are_what_the_table_promises():
    for c in D.CASES:
        t = D.make_inputs(c)
        mem = D.memory_of_rows(c)
        lens = t['lens']
        assert mem.shape == (c.n,) and int(mem.max()) == c.U - 1 and int(mem.min()) == 0
        assert int(lens.max()) == c.Te and (c.U == 1 or int(lens.min()) == 1)
        p = t['prev_att'][:, 0].double()
        assert float((p.sum(-1) - 1).abs().max()) < 1e-6
        for i in range(c.n):
            assert float(p[i, int(lens[mem[i]]):].abs().sum()) == 0.0
        if c.rg > 1 and c.row_mem is None:
            assert torch.equal(mem, torch.arange(c.n) // c.rg)


@pytest.mark.parametrize("case", D.GPU_MULTI + D.SINGLE_CASES, ids=lambda c: c.name)
def test_float32_run_is_far_inside_the_hard_limit(case):
    """e32 of every case and tensor: the float32 CPU run of the same reference (what the sharper bound scales)"""
    t, ref = _base(case)
    r32 = D.reference_of(case, t, dtype=torch.float32)
    e32 = {k: rel_err(r32[k], ref[k]) for k in ref}
    print("DECODESTEP %s | e32 %s" % (case.name, {k: "%.2e" % v for k, v in e32.items()}))
    assert all(0 < v < 1e-5 for v in e32.values()), e32
    for i in range(case.n):
        n = int(t['lens'][D.memory_of_rows(case)[i]])
        assert float(ref['attn'][i, 0, n:].abs().sum()) == 0.0


def _mutations(c, t, attn):
    """name -> the context a defective group kernel would give; attn [n,Te] float64"""
    mem, value, lens = D.memory_of_rows(c), t['value'].double(), t['lens']
    out = {}
    a = attn.clone()
    a[torch.arange(c.n), lens[mem] - 1] = 0                      # the last valid frame left out of the sum
    out['last_frame'] = D.context_per_memory(a, value, mem)
    a = attn.view(c.U, c.rg, c.Te).roll(1, dims=1).reshape(c.n, c.Te)        # the rows of a group rotated by one
    out['rows_rotated'] = D.context_per_memory(a, value, mem)
    out['next_memory'] = D.context_per_memory(attn, value, (mem + 1) % c.U)  # the memory of the next utterance
    if c.Te % 8:
        a = attn.clone()
        a[:, c.Te & ~7:] = 0                                      # the frames of the tail loop left out
        out['tail_frames'] = D.context_per_memory(a, value, mem)
    return out


@pytest.mark.parametrize("case", D.GROUP_CASES, ids=lambda c: c.name)
def test_limit_sees_each_defect_of_the_group_kernel(case):
    t, ref = _base(case)
    moved = {name: rel_err(ctx, ref['ctx']) for name, ctx in _mutations(case, t, ref['attn'][:, 0]).items()}
    print("DECODESTEP %s | ctx shift under mutation %s" % (case.name, {k: "%.2e" % v for k, v in moved.items()}))
    assert (case.Te % 8 != 0) == ('tail_frames' in moved)
    assert all(v > SHIFT for v in moved.values()), moved
    assert SHIFT >= 10 * D.HARD and not math.isnan(sum(moved.values()))


def test_group_cases_cover_the_edges_the_table_names():
    g = {c.name: c for c in D.GROUP_CASES}
    assert set(g) == {'m_rg2_gemm', 'm_rg9_te70', 'm_rg5_te7', 'm_rg16_dv260', 'm_rg32_te512'}
    assert g['m_rg9_te70'].Te > 64 and g['m_rg9_te70'].Te % 8 == 6 and g['m_rg9_te70'].rg % 8 == 1
    assert g['m_rg5_te7'].Te < 8 and g['m_rg5_te7'].Te % 4 and g['m_rg5_te7'].rg < 8
    assert g['m_rg16_dv260'].Dv % 256 == 4 and g['m_rg16_dv260'].n == 512
    assert g['m_rg32_te512'].rg * g['m_rg32_te512'].Te * 4 == 64 * 1024
