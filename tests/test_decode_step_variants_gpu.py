"""GPU: one decode step of speller_ops.SpellerStepper / MultiSpellerStepper (asrk_speller_step_f32, and the many-row
branch: three bf16x6 panel GEMMs + asrk_lstm_cell_fwd_f32) against the float64 reference and on the case table of
tests/decode_step_reference.py - one shape or more per energy-kernel family under row_mem and under shared_kv, per
softmax/context kernel (scalar / vector / row-grouped, the latter on both sides of every condition of its dispatch) and
per cell branch; tests/test_decode_step_plan_cpu.py holds every shape to its kernels.  The attention / decoder modules
are stand-ins with exactly the attributes the steppers read.

Criterion, per output tensor: helpers.rel_err < 1e-3 (the project's hard limit) AND rel_err <= max(F * e32, 4 * 2**-24),
e32 = rel_err of the float32 CPU run of the same reference against its float64 run.  Every test prints e32, the bound,
the device error and device / e32 (pytest -s, lines starting DECODESTEP).  Alignments are exactly 0 beyond the memory's
length and sum to 1 within 1e-5.

F is set per tensor kind to the smallest power of two at least twice the largest device / e32 seen on the MI355X over
every case below (hardware exp in the softmax kernels, 8 waves of partial sums, bf16x6 GEMMs in the gemm branch):

    tensor   largest device / e32   where                                  F
    attn     2.45                   m_rg2_gemm, second step on 16 rows     8
    ctx      1.70                   m_rg2_gemm, second step on 16 rows     4
    h        2.20                   m_rg32_te512                           8
    c        2.31                   m_rg32_te512                           8

(e32 3e-8 ... 5e-7, device 2e-8 ... 1.2e-6; the group kernel and the per-row kernel differ by at most 3e-7 on any output,
and not at all in the alignments of three of the five group cases.)
"""
import ctypes
import importlib
import types

import pytest
import torch

from conftest import PKG_NAME
from helpers import rel_err
import decode_step_reference as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = dict(attn=8, ctx=4, h=8, c=8)
SENTINEL = -12345.678
_cache = {}


def _sops():
    return importlib.import_module(PKG_NAME + ".speller_ops")


def _base(c):
    """inputs, float64 reference and its float32 CPU run of a case: computed once, shared by every test, never
    modified"""
    if c.name not in _cache:
        t = D.make_inputs(c)
        _cache[c.name] = (t, D.reference_of(c, t), D.reference_of(c, t, dtype=torch.float32))
    return _cache[c.name]


def _modules(t, cell):
    ns = types.SimpleNamespace
    p = {k: t[k].to(DEV) for k in D.WEIGHTS}
    att = ns(proj_q=ns(weight=p['Wq'], bias=p['bq']),
             att_layer=ns(loc_conv=ns(weight=p['Wc']), loc_proj=ns(weight=p['Wp']),
                          gen_energy=ns(weight=p['we'], bias=p['be']), temperature=D.TEMPERATURE))
    cellw = (p['W_ih'], p['W_hh'], p['b_ih'], p['b_hh'])
    dec = ns(layers=ns(layer_params=lambda layer: cellw), enable_cell=(cell == 0))
    return att, dec


def _check(label, c, got, ref, r32, rows=None):
    """print every figure, then assert both limits and the alignment-row rule; rows: the first `rows` rows only"""
    t = _base(c)[0]
    bad = []
    for k in ref:
        want, want32 = (ref[k], r32[k]) if rows is None else (ref[k][:rows], r32[k][:rows])
        e32 = rel_err(want32, want)
        err = rel_err(got[k].double().cpu(), want)
        b = D.bound(e32, F[k])
        print("DECODESTEP %s | %s | e32 %.3e | bound %.3e | device %.3e | device/e32 %.2f"
              % (label, k, e32, b, err, err / e32))
        if not (err < D.HARD and err <= b):
            bad.append((k, err, b))
    attn = got['attn'].double().cpu()
    lens = t['lens'][D.memory_of_rows(c)]
    for i in range(attn.shape[0]):
        n = int(lens[i])
        assert float(attn[i, 0, n:].abs().sum()) == 0.0, (label, i)          # exactly 0 beyond the memory's length
        assert abs(float(attn[i, 0, :n].sum()) - 1) < 1e-5, (label, i)
    assert not bad, (label, bad)


# ------------------------------------------------------------------------------------------- MultiSpellerStepper
GUARDED = ('q', 'conv', 'ctx', 'e')


def _multi_stepper(c, t, rg=None):
    """capacity 2 n"""
    att, dec = _modules(t, c.cell)
    return _sops().MultiSpellerStepper(att, dec, t['key'].to(DEV), t['value'].to(DEV), t['lens'].to(DEV), 2 * c.n,
                                       row_group=c.rg if rg is None else rg)


def _guard_intact(st, n):
    want = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    for name in GUARDED:
        tail = getattr(st, name)[n:].contiguous().view(torch.int32)
        assert bool((tail == want).all()), "rows >= n of stepper.%s were written" % name


def _multi_step(ops, st, c, t, n=None, form='plain'):
    """one step on the first n rows, the stepper's per-row buffers filled with a sentinel before it and rows >= n
    holding it afterwards -> dict of device tensors (ctx cloned: it is a view of the stepper's buffer)"""
    n = c.n if n is None else n
    for name in GUARDED:
        getattr(st, name).fill_(SENTINEL)
    d = lambda k: t[k][:n].to(DEV)
    rm = D.row_mem_of(c)[:n].to(torch.int32).to(DEV)
    h, cc = d('h'), d('c')
    if form == 'parent':                         # the entering state is rows parent[i] of a larger, shuffled table
        perm = torch.randperm(n + 3, generator=torch.Generator().manual_seed(1))
        parent = torch.argsort(perm)[:n].to(DEV)                             # table[parent[i]] = state i
        table_h = torch.full((n + 3, c.H), 7.0, device=DEV)
        table_c = torch.full((n + 3, c.H), -7.0, device=DEV)
        table_h[parent], table_c[parent] = h, cc
        out = st.step(rm, d('emb'), d('prev_att'), table_h, table_c, parent=parent)
    elif form == 'state':                        # slot 0 already holds the entering state; h_in / c_in are not read
        hbuf = torch.full((2, n, c.H), SENTINEL, device=DEV)
        cbuf = torch.full((2, n, c.H), SENTINEL, device=DEV)
        hbuf[0], cbuf[0] = h, cc
        out = st.step(rm, d('emb'), d('prev_att'), None, None, state=(hbuf, cbuf))
        assert out[2].data_ptr() == hbuf[1].data_ptr() and out[3].data_ptr() == cbuf[1].data_ptr()
    else:
        out = st.step(rm, d('emb'), d('prev_att'), h, cc)
    ops.check_errors()
    torch.cuda.synchronize()
    _guard_intact(st, n)
    got = dict(attn=out[0], ctx=out[1].clone(), h=out[2])
    if c.cell == 0:
        got['c'] = out[3]
    assert got['attn'].shape == (n, 1, c.Te) and got['ctx'].shape == (n, c.Dv) and got['h'].shape == (n, c.H)
    return got


@pytest.mark.parametrize("case", D.GPU_MULTI, ids=lambda c: c.name)
def test_multi_stepper_vs_float64(ops, case):
    """every MultiSpellerStepper row of the table; rows >= n of the stepper's buffers keep their sentinel bit for bit.
    Group cases also run with row_group = 0 on the same inputs: both pass against float64 independently, and the
    difference between the two kernels is printed."""
    c = case
    t, ref, r32 = _base(c)
    got = _multi_step(ops, _multi_stepper(c, t), c, t)
    _check(c.name, c, got, ref, r32)
    if c.ctx == 'group':
        per_row = _multi_step(ops, _multi_stepper(c, t, rg=0), c, t)
        print("DECODESTEP %s | group kernel - per-row kernel | %s" % (c.name, {
            k: "%.3e" % rel_err(got[k].double().cpu(), per_row[k].double().cpu()) for k in got}))
        _check(c.name + "[row_group=0]", c, per_row, ref, r32)


def test_multi_stepper_reuse_after_the_gemm_branch(ops):
    """one stepper, three steps: all 128 rows (group, gemm: the branch nulls d.Wq for the attention-only call), then
    the first 16 rows (vector, fused: needs Wq back), then all 128 rows again - equal to the first step bit for bit"""
    c = next(c for c in D.CASES if c.name == 'm_rg2_gemm')
    t, ref, r32 = _base(c)
    st = _multi_stepper(c, t)
    first = _multi_step(ops, st, c, t)
    assert st.d.Wq == st.w[0].data_ptr()
    _check(c.name + "[step 1]", c, first, ref, r32)
    few = _multi_step(ops, st, c, t, n=16)
    _check(c.name + "[step 2: 16 rows]", c, few, ref, r32, rows=16)
    again = _multi_step(ops, st, c, t)
    for k in first:
        assert torch.equal(first[k].view(torch.int32), again[k].view(torch.int32)), k


@pytest.mark.parametrize("form", ["parent", "state"])
@pytest.mark.parametrize("name", ["m_perm", "m_rg2_gemm"])
def test_multi_stepper_entry_forms(ops, name, form):
    """parent= (the gather lands in the state slot) and state= (slot 0 pre-filled) give what the plain form gives, in
    the fused and in the gemm branch"""
    c = next(c for c in D.CASES if c.name == name)
    t, ref, r32 = _base(c)
    got = _multi_step(ops, _multi_stepper(c, t), c, t, form=form)
    _check("%s[%s]" % (c.name, form), c, got, ref, r32)


def test_multi_stepper_capacity_overflow(ops):
    lib = importlib.import_module(PKG_NAME + "._lib")
    c = next(c for c in D.CASES if c.name == 'm_perm')
    t = _base(c)[0]
    att, dec = _modules(t, c.cell)
    st = _sops().MultiSpellerStepper(att, dec, t['key'].to(DEV), t['value'].to(DEV), t['lens'].to(DEV), c.n - 1)
    d = lambda k: t[k].to(DEV)
    with pytest.raises(lib.AsrkError):
        st.step(D.row_mem_of(c).to(torch.int32).to(DEV), d('emb'), d('prev_att'), d('h'), d('c'))


# ------------------------------------------------------------------------------------------------ SpellerStepper
def _single_stepper(c, t):
    att, dec = _modules(t, c.cell)
    return _sops().SpellerStepper(att, dec, t['key'].to(DEV), t['value'].to(DEV), t['lens'].to(DEV), c.n,
                                  shared=(c.stepper == 'shared'))


def _single_step(ops, st, c, emb, prev_att):
    out = st.step(emb.to(DEV), prev_att.to(DEV))
    ops.check_errors()
    torch.cuda.synchronize()
    got = dict(attn=out[0].clone(), ctx=out[1].clone(), h=out[2].clone())      # views the next call overwrites
    if c.cell == 0:
        got['c'] = out[3].clone()
    assert got['attn'].shape == (c.n, 1, c.Te) and got['ctx'].shape == (c.n, c.Dv) and got['h'].shape == (c.n, c.H)
    return got


@pytest.mark.parametrize("case", D.SINGLE_CASES, ids=lambda c: c.name)
def test_single_stepper_vs_float64(ops, case):
    """shared_kv = 1 with 1 and 16 rows in both energy-kernel families and both cells, one memory per row with ragged
    lengths, and (s_chain) two chained steps: state slot 1 -> slot 0, prev_att = the first step's alignment"""
    c = case
    t, ref, r32 = _base(c)
    st = _single_stepper(c, t)
    st.h[0].copy_(t['h'].to(DEV))
    st.c[0].copy_(t['c'].to(DEV))
    got = _single_step(ops, st, c, t['emb'], t['prev_att'])
    _check(c.name, c, got, ref, r32)
    if c.steps == 2:
        emb2 = t['emb'].flip(0).contiguous() * 0.5
        over = lambda r: dict(emb=emb2, prev_att=r['attn'], h=r['h'], c=r.get('c', t['c']))
        ref2 = D.reference_of(c, t, **over(ref))
        r32_2 = D.reference_of(c, t, dtype=torch.float32, **over(r32))
        st.h[0].copy_(st.h[1])
        st.c[0].copy_(st.c[1])
        got2 = _single_step(ops, st, c, emb2, got['attn'])
        _check(c.name + "[step 2]", c, got2, ref2, r32_2)
        assert rel_err(got2['h'].cpu(), got['h'].cpu()) > 1e-2            # the second step did move the state


def test_step_refuses_unsupported_descriptors(ops):
    """several heads, dot-product attention or a stacked decoder: asrk_speller_step_f32 answers ASRK_ESHAPE (raised as
    AsrkError) and computes nothing"""
    lib = importlib.import_module(PKG_NAME + "._lib")
    L = lib.load()
    c = next(c for c in D.CASES if c.name == 's_rows3')
    t = _base(c)[0]
    st = _single_stepper(c, t)
    st.h[0].copy_(t['h'].to(DEV))
    st.c[0].copy_(t['c'].to(DEV))
    outputs = (st.q, st.conv, st.attn, st.ctx, st.e, st.h[1], st.c[1])
    for o in outputs:
        o.fill_(SENTINEL)
    emb, prev = t['emb'].to(DEV), t['prev_att'].to(DEV)
    for field, value in (('nhead', 2), ('att_mode', 1), ('nlayer', 2)):
        keep = getattr(st.d, field)
        setattr(st.d, field, value)
        try:
            rc = L.asrk_speller_step_f32(ctypes.byref(st.d), 0, ctypes.c_void_p(prev.data_ptr()), c.Te,
                                         ctypes.c_void_p(emb.data_ptr()), ops._stream())
            assert rc == -2, (field, rc)
            with pytest.raises(lib.AsrkError):
                st.step(emb, prev)
        finally:
            setattr(st.d, field, keep)
    torch.cuda.synchronize()
    want = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    for o in outputs:
        assert bool((o.contiguous().view(torch.int32) == want).all())
    got = _single_step(ops, st, c, t['emb'], t['prev_att'])                 # the descriptor is whole again
    _check(c.name + "[after refusals]", c, got, _base(c)[1], _base(c)[2])
